#!/usr/bin/env python3
"""Batch means and the mean test (include/mcmcref_bm.h): time per kernel and per step, beside the project's streaming
yardsticks and numpy for the same work.

    python tools/batchmeans_bench.py [--out profiles/batch_means.json] [--runs 9]

Workloads: 4 chains x 10 000 draws x 100 parameters, f64, in both layouts ([P][C][N]: k_bm_time; the sampler's [C][N][P]:
k_bm_tile), and 4 x 100 000 x 16 in [P][C][N].  The draws are resident on the device.  Per workload, at the default lugsail
batch size b and at b / 3: the streaming kernel's time from the library's own HIP events (`batchmeans.kernel_ms`) and its
read rate (bytes of draws / time); `Context.hbm_probe`'s read rate over a buffer of the same size in the same run; the time
of `Context.moments` on the same tensor -- the project's streaming kernel, one pass for mean and std -- both as the sum
of its kernels' HIP-event times (`Context.profile_get`) and as a host clock around the synchronous call; and
the whole `mean_shift_test` of the tensor against itself, split into its steps by host clocks around the synchronous
entries: batch means (four passes: b and b / 3 of both samples), the pooled copies, the covariances (four of batch means,
two of the pooled draws for the two mESS), finish and pool, Cholesky and solve.  Every figure is the median of `--runs`
runs; the runs of the workloads alternate (run r of every workload before run r + 1 of any) so that drift hits all alike.
numpy does the same test on the host with the thread count of the environment (reported).
"""
import argparse, json, os, statistics, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, batchmeans

STAGES = ("batch_means", "pooled", "covariance", "finish_pool", "cholesky", "solve")


def ar1(C, N, P, phi, seed):
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    return lfilter([1.0], [1.0, -phi], rng.standard_normal((P, C, N)), axis=2)


def numpy_route(x, b):
    """The mean test of x [P][C][N] against itself in numpy: lugsail batch means, sample covariances, solve."""
    P, C, N = x.shape

    def sigma(bb):
        a = N // bb
        m = x[:, :, N - a * bb:].reshape(P, C, a, bb).mean(axis=3).reshape(P, C * a)
        return np.cov(m, ddof=0) * bb * (C * a) / (C * a - 1)

    sig = 2 * sigma(b) - sigma(b // 3)
    lam = np.cov(x.reshape(P, -1), ddof=0)
    mess = C * N * np.exp((np.linalg.slogdet(lam)[1] - np.linalg.slogdet(sig)[1]) / P)
    V = 2 * sig / (C * (N // b) * b)
    d = np.zeros(P)
    return float(d @ np.linalg.solve(V, d)), mess


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=9)
a = ap.parse_args()
ctx = _ffi.Context(0)
work = []
for name, (C, N, P), layout in (("4x10000x100 pcn", (4, 10000, 100), "pcn"), ("4x10000x100 cnp", (4, 10000, 100), "cnp"),
                                ("4x100000x16 pcn", (4, 100000, 16), "pcn")):
    x = ar1(C, N, P, 0.9, seed=N + P)
    arr = x if layout == "pcn" else np.ascontiguousarray(x.transpose(1, 2, 0))
    t = ctx.upload(arr, layout)
    b = batchmeans.batch_size(N, 3)[0]
    got, want = batchmeans.batch_means(t, batch=b, context=ctx), batchmeans.batch_means_host(arr, layout, batch=b)
    assert np.array_equal(got["bm"].view(np.int64), want["bm"].view(np.int64)) and np.array_equal(got["mu"].view(np.int64), want["mu"].view(np.int64))
    work.append({"name": name, "x": x, "t": t, "b": b, "layout": layout, "bytes": arr.nbytes, "route": "time" if layout == "pcn" else "tile",
                 "route_b": [], "route_b3": [], "mean_b": [], "moments": [], "moments_kernels": [], "info": None, "mess": None, "test": [], "numpy": [], **{s: [] for s in STAGES}})
batchmeans.profile(True, ctx)
for run in range(a.runs + 1):                                          # run 0 warms up
    for w in work:
        for key, bb in (("route_b", w["b"]), ("route_b3", w["b"] // 3)):
            batchmeans.batch_means(w["t"], batch=bb, context=ctx)
            ms = batchmeans.kernel_ms(ctx)
            if run:
                w[key].append(ms[w["route"]])
                if key == "route_b":
                    w["mean_b"].append(ms["mean"])
        t0 = time.perf_counter()
        ctx.moments(w["t"])
        dt = time.perf_counter() - t0
        if run:
            w["moments"].append(dt * 1e3)
batchmeans.profile(False, ctx)
ctx.profile(True)
for run in range(a.runs + 1):
    for w in work:
        ctx.profile_reset()
        ctx.moments(w["t"])
        if run:
            w["moments_kernels"].append(sum(k["total_ms"] for k in ctx.profile_get().values()))
ctx.profile(False)
for run in range(a.runs + 1):
    for w in work:
        stages = {}
        t0 = time.perf_counter()
        res = batchmeans.mean_shift_test(w["t"], w["t"], context=ctx, stages=stages)
        dt = time.perf_counter() - t0
        w["info"], w["mess"] = res["info"], res["mess_ref"]
        if run:
            w["test"].append(dt * 1e3)
            for s in STAGES:
                w[s].append(stages.get(s, 0.0) * 1e3)
for run in range(3):
    for w in work:
        t0 = time.perf_counter()
        numpy_route(w["x"], w["b"])
        w["numpy"].append((time.perf_counter() - t0) * 1e3)
rows = []
for w in work:
    med = {k: statistics.median(w[k]) for k in ("route_b", "route_b3", "mean_b", "moments", "moments_kernels", "test", "numpy") + STAGES}
    probe = ctx.hbm_probe(max(w["bytes"], 1 << 20), 9)
    rows.append({"workload": w["name"], "kernel": "k_bm_" + w["route"], "batch": w["b"], "draw_bytes": w["bytes"],
                 "kernel_ms_b": med["route_b"], "kernel_ms_b3": med["route_b3"], "mean_kernel_ms": med["mean_b"],
                 "kernel_read_GBps_b": w["bytes"] / (med["route_b"] * 1e-3) / 1e9,
                 "kernel_read_GBps_b3": w["bytes"] / (med["route_b3"] * 1e-3) / 1e9,
                 "hbm_probe_read_GBps_same_size": probe["read_GBps"], "moments_call_ms": med["moments"],
                 "moments_kernels_ms": med["moments_kernels"], "moments_kernels_GBps": w["bytes"] / (med["moments_kernels"] * 1e-3) / 1e9,
                 "mean_shift_test_ms": med["test"], "mean_shift_test_info": w["info"], "mess": w["mess"] if w["mess"] == w["mess"] else None,
                 "steps_ms": {s: med[s] for s in STAGES}, "numpy_ms": med["numpy"], "numpy_runs": 3})
    print(json.dumps(rows[-1]), flush=True)
out = {"runs": a.runs, "hbm_probe_1GiB_read_GBps": ctx.hbm_probe(1 << 30, 5)["read_GBps"],
       "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None, "workloads": rows}
print(json.dumps({k: v for k, v in out.items() if k != "workloads"}))
if a.out:
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
ctx.close()

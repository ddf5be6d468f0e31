#!/usr/bin/env python3
"""Sliced two-sample KS / Wasserstein-1 (mcr_sliced_two_sample_dev): what the projection kernel and the whole call cost.

    python tools/sliced_bench.py [--reps 9] [--host-reps 3] [--out profiles/sliced_two_sample.json]

Workload: a reference of 4 chains x 10 000 draws x 100 parameters against an actual sample of the same shape, K = 64
directions (`validate.sliced_directions` on the reference's std, centre = its means), both samples resident on the
device.  After one warm-up, median and range of `reps` runs of

1. the HIP-event time of k_project, both launches of a call together and per launch (profiled runs of their own: the
   events cost the whole call a little),
2. k_project's effective bytes/s, (P + K) M 8 bytes per launch -- X read once, Z written once; the re-reads of X by the
   K / MCR_PROJ_TILE_K direction tiles are not counted -- beside mcr_hbm_probe's read rate on the same device,
3. the whole mcr_sliced_two_sample_dev call on the host clock (unprofiled), and its other kernels' event times,
4. for context only, the host route: numpy `W @ (X - c)` plus scipy.stats.ks_2samp / wasserstein_distance per direction
   (`host-reps` runs).

Before anything is timed the device's KS is compared with scipy's on every direction (1e-12 relative; the exact tests
are tests/test_sliced_gpu.py)."""
import argparse, json, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402
from mcmc_ref_hip.validate import sliced_directions  # noqa: E402

C_, N, P, K = 4, 10_000, 100, 64


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def host_route(ref, act, W, center):
    from scipy.stats import ks_2samp, wasserstein_distance
    t0 = time.perf_counter()
    zr, za = W @ (ref - center[:, None]), W @ (act - center[:, None])
    t1 = time.perf_counter()
    ks = np.array([ks_2samp(r, a).statistic for r, a in zip(zr, za)])
    w1 = np.array([wasserstein_distance(r, a) for r, a in zip(zr, za)])
    t2 = time.perf_counter()
    return ks, w1, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sliced_two_sample.json"))
    a = ap.parse_args()
    M = C_ * N
    rng = np.random.default_rng(4711)
    scale, loc = 10.0 ** rng.integers(-2, 3, size=P), rng.normal(size=P) * 10.0
    ref = loc[:, None] + scale[:, None] * rng.normal(size=(P, M))
    act = loc[:, None] + scale[:, None] * (0.05 + 1.1 * rng.normal(size=(P, M)))
    center = ref.mean(axis=1)
    W, live = sliced_directions(K, ref.std(axis=1))
    assert live.all()
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "directions": K, "pooled_draws": M},
           "reps": a.reps, "tile": {"M": _ffi.MCR_PROJ_TILE_M, "K": _ffi.MCR_PROJ_TILE_K, "chunk_P": _ffi.MCR_PROJ_CHUNK_P}}
    with _ffi.Context(0) as ctx:
        out["hbm_read_GBps"] = round(ctx.hbm_probe(1 << 30, 3)["read_GBps"], 1)
        dr = _ffi.DeviceBuffer(ctx, ref.nbytes).upload(ref)
        da = _ffi.DeviceBuffer(ctx, act.nbytes).upload(act)
        call = lambda: ctx.sliced_two_sample_dev(dr.ptr, M, da.ptr, M, P, W, center)
        out["directions_per_chunk"] = ctx.sliced_dirs_per_chunk(M, M, P, K)
        ks, w1 = call()                                               # warm-up, and the check
        hks, hw1, _, _ = host_route(ref, act, W, center)
        out["max_rel_ks_difference_from_scipy"] = float(np.max(np.abs(ks - hks) / hks))
        out["max_rel_w1_difference_from_scipy"] = float(np.max(np.abs(w1 - hw1) / hw1))
        assert out["max_rel_ks_difference_from_scipy"] < 1e-12 and out["max_rel_w1_difference_from_scipy"] < 1e-9
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        proj, others = [], {}
        for _ in range(a.reps):
            ctx.profile_reset()
            call()
            pr = ctx.profile_get()
            assert pr["k_project"]["launches"] == 2 * -(-K // out["directions_per_chunk"])
            proj.append(pr["k_project"]["total_ms"])
            for k, v in pr.items():
                if k != "k_project" and v["launches"]:
                    others.setdefault(k, []).append(v["total_ms"])
        ctx.profile(False)
        ctx.profile_reset()
        dr.free()
        da.free()
    launches = 2 * -(-K // out["directions_per_chunk"])
    per_launch = [t / launches for t in proj]
    nbytes = (P + K) * M * 8
    out["k_project_per_call"] = {"launches": launches, **spread(proj)}
    out["k_project_per_launch"] = spread(per_launch)
    out["k_project_effective_GBps"] = round(nbytes / statistics.median(per_launch) / 1e6, 1)
    out["k_project_bytes_per_launch"] = nbytes
    out["k_project_x_reads_per_launch"] = -(-K // _ffi.MCR_PROJ_TILE_K)
    out["k_project_GFLOPs"] = round(2.0 * K * P * M / statistics.median(per_launch) / 1e6, 1)
    out["k_project_frac_of_hbm_read"] = round(out["k_project_effective_GBps"] / out["hbm_read_GBps"], 3)
    out["call"] = spread(wall, 3)
    out["other_kernels_ms_median_per_call"] = {k: round(statistics.median(v), 4) for k, v in sorted(others.items())}
    hp, hs = [], []
    for _ in range(a.host_reps):
        _, _, p_ms, s_ms = host_route(ref, act, W, center)
        hp.append(p_ms)
        hs.append(s_ms)
    out["host_route_context_only"] = {"reps": a.host_reps, "numpy_projection": spread(hp, 2), "scipy_ks_w1": spread(hs, 2)}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

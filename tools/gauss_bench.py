#!/usr/bin/env python3
"""Dense Cholesky, lower solve and the joint Gaussian check (include/mcmcref_hip_ext.h): time per call and per kernel.

    python tools/gauss_bench.py [--out gauss.json] [--reps 5] [--sizes 128,1024,4096]

Per order P: `gaussian.cholesky_dev` on a matrix of condition 1e3 (checked first: info 0 and the entrywise residual
|A - L L^T| <= gamma_{P+1} |L| |L|^T of tests/test_gaussian_refs_cpu.py, in double here, so the figure printed is the
ratio plus numpy's own rounding) and `gaussian.solve_lower_dev` with K = P right-hand sides; `flops` prices them at
P^3 / 3 and P^2 K multiply-adds.  Then `gaussian.gaussian_check_dev` at the shapes validate() sees, beside
`Context.energy_distance_dev` on the same draws thinned to 4 000 a side: the two joint checks' cost side by side.
Kernel times come from the library's profiling events (one event pair per launch), call times from the host clock
around synchronous calls, each the mean of `--reps` calls after one warm-up call.
"""
import argparse, json, sys, time
from pathlib import Path
import numpy as np
ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi, _xabi, gaussian

U = 2.0 ** -53


def spd(P, cond, rng):
    Q = np.linalg.qr(rng.standard_normal((P, P)))[0]
    A = (Q * np.logspace(0.0, -np.log10(cond), P)) @ Q.T
    return (A + A.T) / 2


def timed(ctx, call, reps, restore=None):
    """(mean call ms, {kernel: (launches per call, ms per call)}) of `call`, after one warm-up call."""
    call()
    ctx.profile(True); ctx.profile_reset()
    wall = 0.0
    for _ in range(reps):
        if restore:
            restore()
        t0 = time.perf_counter()
        call()
        wall += time.perf_counter() - t0
    pr = ctx.profile_get(); ctx.profile(False)
    return wall / reps * 1e3, {k: (v["launches"] / reps, v["total_ms"] / reps) for k, v in pr.items()}


ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="128,512,1024,2048,4096,8192")
a = ap.parse_args()
ctx = _ffi.Context(0)
rows = []
for P in (int(s) for s in a.sizes.split(",")):
    rng = np.random.default_rng(P)
    A = spd(P, 1e3, rng)
    da = _ffi.DeviceBuffer(ctx, A.nbytes).upload(A)
    info, logdet = gaussian.cholesky_dev(da.ptr, P, context=ctx)
    L = da.download(np.float64, P * P).reshape(P, P)
    assert info == 0 and not np.triu(L, 1).any()
    res = np.abs(A - L @ L.T)
    bound = (P + 1) * U / (1 - (P + 1) * U) * (np.abs(L) @ np.abs(L).T)
    ratio = float((res / bound)[np.tril_indices(P)].max())
    ld_err = abs(logdet - 2 * np.log(np.diag(L)).sum())
    assert ratio <= 1.0 and ld_err <= 1e-13 * (np.abs(2 * np.log(np.diag(L))).sum() + 1), (P, ratio, ld_err)
    chol_ms, chol_k = timed(ctx, lambda: gaussian.cholesky_dev(da.ptr, P, context=ctx), a.reps, restore=lambda: da.upload(A))
    B = rng.standard_normal((P, P))
    dl, db = _ffi.DeviceBuffer(ctx, L.nbytes).upload(L), _ffi.DeviceBuffer(ctx, B.nbytes).upload(B)
    gaussian.solve_lower_dev(dl.ptr, P, db.ptr, P, context=ctx)
    X = db.download(np.float64, P * P).reshape(P, P)
    sres = np.abs(L @ X - B)
    sbound = P * U / (1 - P * U) * (np.abs(L) @ np.abs(X))
    sratio = float((sres / sbound).max())
    assert sratio <= 1.0, (P, sratio)
    solve_ms, solve_k = timed(ctx, lambda: gaussian.solve_lower_dev(dl.ptr, P, db.ptr, P, context=ctx), a.reps,
                              restore=lambda: db.upload(B))
    kern = lambda d: sum(ms for _, ms in d.values())
    rows.append({"P": P, "cholesky_call_ms": chol_ms, "cholesky_kernels_ms": kern(chol_k),
                 "cholesky_launches": sum(n for n, _ in chol_k.values()),
                 "cholesky_GFLOPs": 2 * P ** 3 / 3 / (kern(chol_k) * 1e-3) / 1e9, "cholesky_residual_over_bound": ratio,
                 "cholesky_by_kernel_ms": {k: ms for k, (_, ms) in chol_k.items()},
                 "solve_call_ms": solve_ms, "solve_kernel_ms": kern(solve_k), "solve_GFLOPs": 2 * P ** 3 / 2 / (kern(solve_k) * 1e-3) / 1e9,
                 "solve_residual_over_bound": sratio})
    print(json.dumps(rows[-1]), flush=True)
    for d in (da, dl, db):
        d.free()
checks = []
for P, M in ((10, 40000), (100, 40000), (400, 40000)):
    rng = np.random.default_rng(P)
    mix = rng.standard_normal((P, P)) / np.sqrt(P) + np.eye(P)
    ref, act = mix @ rng.standard_normal((P, M)), mix @ rng.standard_normal((P, M))
    scale = 1.0 / ref.std(axis=1)
    dr, dact = _ffi.DeviceBuffer(ctx, ref.nbytes).upload(ref), _ffi.DeviceBuffer(ctx, act.nbytes).upload(act)
    r = gaussian.gaussian_check_dev(dr.ptr, M, dact.ptr, M, P, scale=scale, context=ctx)
    # two samples of one Gaussian: kl_sym is about P (P + 3) / 2 (1 / Mr + 1 / Ma), the estimation noise of the P (P + 3) / 2 moments
    expect = P * (P + 3) / 2 * (2.0 / M)
    assert r["info_ref"] == 0 and r["info_act"] == 0 and expect / 2 < r["kl_sym"] < 2 * expect, (r, expect)
    g_ms, g_k = timed(ctx, lambda: gaussian.gaussian_check_dev(dr.ptr, M, dact.ptr, M, P, scale=scale, context=ctx), a.reps)
    thin = np.ascontiguousarray(ref[:, ::10]), np.ascontiguousarray(act[:, ::10])
    tr, ta = _ffi.DeviceBuffer(ctx, thin[0].nbytes).upload(thin[0]), _ffi.DeviceBuffer(ctx, thin[1].nbytes).upload(thin[1])
    e_ms, _ = timed(ctx, lambda: ctx.energy_distance_dev(tr.ptr, M // 10, ta.ptr, M // 10, P, scale), a.reps)
    checks.append({"P": P, "M": M, "gaussian_check_call_ms": g_ms, "gaussian_check_launches": sum(n for n, _ in g_k.values()),
                   "gaussian_check_by_kernel_ms": {k: ms for k, (_, ms) in g_k.items()}, "kl_sym": r["kl_sym"],
                   "mahalanobis": r["mahalanobis"], "energy_distance_4000_draws_call_ms": e_ms})
    print(json.dumps(checks[-1]), flush=True)
    for d in (dr, dact, tr, ta):
        d.free()
out = {"block": _xabi.MCRX_CHOL_NB, "factorisation": rows, "gaussian_check": checks}
if a.out:
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
ctx.close()

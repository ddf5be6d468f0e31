#!/usr/bin/env python3
"""PSIS-LOO (mcr_psis_dev): what the two new kernels and the whole call cost, next to the sort stage they reuse.

    python tools/psis_bench.py [--reps 9] [--out profiles/psis.json]

Workloads, f64, resident on the device: 4 chains x 1 000 draws x 10 000 observations (a LOO-sized model) and 4 x 10 000 x
100, pointwise log-likelihoods of normal observations (negate = 1).  Per workload, after one warm-up of both calls (three
columns are checked against the library's host routine),

1. the whole call WITHOUT and WITH the log weights (they stay in device memory) on the host clock, ALTERNATING, median /
   min / max of `reps` unprofiled runs each,
2. the HIP-event time of every kernel of a call with weights (`Context.profile`, runs of their own: the events cost a
   little),
3. k_psis_column and k_psis_weights against the sort stage they follow (every other kernel of the call but k_finalize),
   and k_psis_column's effective read rate: the 8 M bytes of a column's keys over its time (the passes after the first
   are served by L2 and LDS, so this is the rate at which columns are consumed, not a memory rate).
"""
import argparse, ctypes as C, json, math, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

SHAPES = ((4, 1_000, 10_000), (4, 10_000, 100))


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def log_lik(C_, N, P, seed=4711):
    """[P][C][N] log-likelihoods of P normal observations under C N posterior draws of their mean."""
    rng = np.random.default_rng(seed)
    y = rng.normal(size=(P, 1)).astype(np.float64)
    mu = rng.normal(scale=0.3, size=(1, C_ * N))
    return (-0.5 * ((y - mu) ** 2 + math.log(2.0 * math.pi))).reshape(P, C_, N)


def measure(ctx, C_, N, P, reps):
    M = C_ * N
    x = log_lik(C_, N, P)
    t = ctx.upload(x)
    wbuf = _ffi.DeviceBuffer(ctx, P * M * 8)
    arrs = {n: np.full(P, np.nan) for n in ("khat", "lppd", "elpd", "p_loo")}
    nt = np.zeros(P, dtype=np.int64)

    def call(weights):
        out = _ffi.Psis(ndraws_tail=_ffi._as_ip(nt), log_weights=wbuf.ptr if weights else None,
                        **{n: _ffi._as_dp(a) for n, a in arrs.items()})
        ctx._check(ctx.lib.mcr_psis_dev(ctx.handle, t.buf.ptr, *t.targs, 1, None, None, C.byref(out)))

    out = {"workload": {"chains": C_, "draws_per_chain": N, "observations": P, "pooled_draws": M, "dtype": "f64"},
           "columns_per_chunk": ctx.psis_params_per_chunk(t)}
    call(True)                                                    # warm-up, and the check
    call(False)
    lw = wbuf.download(np.float64, P * M).reshape(P, M)
    for p in (0, P // 2, P - 1):
        h = _ffi.psis_host(x[p].reshape(-1), negate=True)
        assert h["ndraws_tail"] == nt[p] and abs(arrs["khat"][p] - h["khat"]) <= 1e-9 and abs(arrs["elpd"][p] - h["elpd"]) <= 1e-9
        assert np.max(np.abs(lw[p] - h["log_weights"])) <= 1e-9 * max(1.0, np.max(np.abs(h["log_weights"])))
    del lw
    wall = {"without_weights": [], "with_weights": []}
    for _ in range(reps):                                         # alternating
        for name, w in (("without_weights", False), ("with_weights", True)):
            t0 = time.perf_counter()
            call(w)
            wall[name].append((time.perf_counter() - t0) * 1e3)
    ctx.profile(True)
    kern = {}
    for _ in range(reps):
        ctx.profile_reset()
        call(True)
        for k, v in ctx.profile_get().items():
            if v["launches"]:
                kern.setdefault(k, []).append(v["total_ms"])
    ctx.profile(False)
    ctx.profile_reset()
    wbuf.free()
    t.free()
    med = {k: statistics.median(v) for k, v in kern.items()}
    col, wts = med["k_psis_column"], med["k_psis_weights"]
    sort = sum(v for k, v in med.items() if k not in ("k_psis_column", "k_psis_weights", "k_finalize"))
    out.update({"ndraws_tail": int(nt[0]), "elpd_loo": math.fsum(arrs["elpd"]),
                "call": {k: spread(v, 3) for k, v in wall.items()},
                "kernels_ms_per_call": {k: spread(v) for k, v in sorted(kern.items())},
                "sort_stage_ms": round(sort, 4),
                "k_psis_column_over_sort_stage": round(col / sort, 3), "k_psis_weights_over_sort_stage": round(wts / sort, 3),
                "k_psis_column_keys_GB_per_s": round(8.0 * P * M / col / 1e6, 1),
                "with_weights_over_without": round(statistics.median(wall["with_weights"]) /
                                                   statistics.median(wall["without_weights"]), 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "psis.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "threads_per_column": 256, "shapes": []}
    with _ffi.Context(0) as ctx:
        for C_, N, P in SHAPES:
            out["shapes"].append(measure(ctx, C_, N, P, a.reps))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

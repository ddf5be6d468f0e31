#!/usr/bin/env python3
"""Nested R-hat (mcr_nested_rhat_dev): what the two new kernels and the whole call cost.

    python tools/nested_bench.py [--reps 9] [--out profiles/nested_rhat.json]

Workload: 4096 chains x 100 draws x 100 parameters, f64, resident on the device, K = 64 superchains of 64 chains.
After one warm-up (which is also checked against a numpy restatement of the raw kind),

1. the whole call on the host clock, median / min / max of `reps` unprofiled runs,
2. the HIP-event time of every kernel of a call (`Context.profile`, runs of their own: the events cost a little),
3. k_chain_moments' effective bytes/s over its compulsory bytes -- 16 bytes per draw (x, and the two 4-byte codes) plus
   the 2 M-double z table once -- as a fraction of the HBM read rate profiles/sliced_two_sample.json records (and of
   mcr_hbm_probe's rate on this device, measured here),
4. the share of the kernel time spent in the two new kernels against the reused sort and fold stages.
"""
import argparse, json, statistics, sys, time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

C_, N, P, K = 4096, 100, 100, 64
NEW = ("k_chain_moments", "k_nested_combine")
FOLD = ("k_fold_merge",)


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def raw_reference(x, ids):
    """nrhat_raw of x[C][N] in numpy (two-pass, float64)."""
    m = x.mean(axis=1)
    q = ((x - m[:, None]) ** 2).sum(axis=1)
    L = x.shape[0] // K
    mu_k = np.array([m[ids == g].mean() for g in range(K)])
    t_k = np.array([((m[ids == g] - mu_k[g]) ** 2).sum() / (L - 1) + q[ids == g].sum() / (L * (x.shape[1] - 1)) for g in range(K)])
    return float(np.sqrt(1.0 + mu_k.var(ddof=1) / t_k.mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "nested_rhat.json"))
    a = ap.parse_args()
    M = C_ * N
    rng = np.random.default_rng(4711)
    x = rng.normal(size=(P, C_, N)) * (10.0 ** rng.integers(-2, 3, size=(P, 1, 1))) + rng.normal(size=(P, 1, 1))
    ids = np.repeat(np.arange(K, dtype=np.int32), C_ // K)
    recorded = json.loads((ROOT / "profiles" / "sliced_two_sample.json").read_text())["hbm_read_GBps"]
    out = {"workload": {"chains": C_, "draws_per_chain": N, "parameters": P, "superchains": K, "pooled_draws": M, "dtype": "f64"},
           "reps": a.reps, "register_block": _ffi.MCR_NESTED_BLOCK, "hbm_read_GBps_recorded": recorded}
    with _ffi.Context(0) as ctx:
        out["hbm_read_GBps_here"] = round(ctx.hbm_probe(1 << 30, 3)["read_GBps"], 1)
        t = ctx.upload(x)
        out["parameters_per_chunk"] = ctx.nested_params_per_chunk(t, K)
        call = lambda: ctx.nested_rhat(t, ids)
        got = call()                                                  # warm-up, and the check
        for p in (0, P // 2, P - 1):
            want = raw_reference(x[p], ids)
            assert abs(got["nrhat_raw"][p] - want) <= 1e-9 * want, (p, got["nrhat_raw"][p], want)
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        kern = {}
        for _ in range(a.reps):
            ctx.profile_reset()
            call()
            for k, v in ctx.profile_get().items():
                if v["launches"]:
                    kern.setdefault(k, []).append(v["total_ms"])
        ctx.profile(False)
        ctx.profile_reset()
        t.free()
    chunks = -(-P // out["parameters_per_chunk"])
    med = {k: statistics.median(v) for k, v in kern.items()}
    total = sum(med.values())
    nbytes = P * M * 16 + chunks * 2 * M * 8
    mom = med["k_chain_moments"]
    out["call"] = spread(wall, 3)
    out["kernels_ms_per_call"] = {k: spread(v) for k, v in sorted(kern.items())}
    out["k_chain_moments_bytes_per_call"] = nbytes
    out["k_chain_moments_effective_GBps"] = round(nbytes / mom / 1e6, 1)
    out["k_chain_moments_frac_of_hbm_read"] = round(nbytes / mom / 1e6 / recorded, 3)
    out["k_chain_moments_frac_of_hbm_read_here"] = round(nbytes / mom / 1e6 / out["hbm_read_GBps_here"], 3)
    new = sum(med[k] for k in NEW)
    fold = sum(med.get(k, 0.0) for k in FOLD)
    sort = total - new - fold - med.get("k_finalize", 0.0)
    out["share_of_kernel_time"] = {"new_kernels": round(new / total, 3), "sort_stage": round(sort / total, 3),
                                   "fold_stage": round(fold / total, 3), "kernel_ms_total": round(total, 4)}
    out["new_kernels_over_sort_stage"] = round(new / sort, 3)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Energy distance (mcr_energy_distance_dev): what the call and its two kernels cost, next to scipy's cdist and to the fp64
vector peak.

    python tools/energy_bench.py [--reps 9] [--out profiles/energy_distance.json]

Shapes, f64, resident on the device: 4 x 10 000 x 100 against itself (the flagship shape: 40 000 draws a side), 4 x 1 000
x 10 against itself, and the 2 x 2 000 / 2 x 2 037 separation case of the tests.  Per shape, after a warm-up whose result
is checked against the library's host routine (on the first 2 000 draws a side where the whole is too large for the host),

1. the whole call on the host clock (it ends in a synchronise) ALTERNATING with the baseline: the same three pair sums by
   scipy.spatial.distance.cdist in blocks of 1 000 rows on 16 threads, without the symmetry of the two within-sample sums
   (using it would at most halve two of the three).  Median / min / max of `reps` runs each.  Where 2 Mr Ma P is more
   than 2e9 the baseline runs on every k-th draw and its time is scaled by the ratio of the pair counts: the JSON says so.
2. the HIP-event time of both kernels (`Context.profile`, runs of their own) and k_energy_pairs' launches.  The launches
   of a call carry the same number of tiles (+-1) and every tile costs the same, so the longest launch is the kernel's time
   over its launches.
3. k_energy_pairs against its VALU bound: 2 fp64 vector operations (a subtract, an fma) per pair-parameter, the 78.6
   TFLOP/s vector peak = 39.3e12 such operations a second; counted over the pair-parameters the sums need, (Mr Ma + Mr (Mr + 1) / 2 + Ma (Ma + 1) / 2) P, not over the
   tiles' padding.

Then the worst relative errors of the device against the host routine over the tile and chunk edges the tests use.
"""
import argparse, json, statistics, sys, time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "mcmc-db_amd")]
from mcmc_ref_hip import _ffi  # noqa: E402

VALU_OPS_PER_S = 39.3e12          # fp64 vector operations a second at the 78.6 TFLOP/s vector peak (an fma counts as two flops)
THREADS, BLOCK, BASELINE_WORK = 16, 1000, 2e9


def spread(ms, digits=4):
    return {"median_ms": round(statistics.median(ms), digits), "min_ms": round(min(ms), digits), "max_ms": round(max(ms), digits)}


def separation_case():
    rng = np.random.default_rng(0)
    plus = np.linalg.cholesky(np.array([[1.0, 0.9], [0.9, 1.0]]))
    minus = np.linalg.cholesky(np.array([[1.0, -0.9], [-0.9, 1.0]]))
    ref = plus @ rng.normal(size=(2, 2000))
    actual = minus @ rng.normal(size=(2, 2037))
    return ref, actual


def shapes():
    rng = np.random.default_rng(4711)
    big = rng.normal(size=(100, 40_000)) * rng.uniform(0.5, 20.0, size=(100, 1))
    small = rng.normal(size=(10, 4_000)) * rng.uniform(0.5, 20.0, size=(10, 1))
    yield "4 x 10000 x 100 against itself", big, big
    yield "4 x 1000 x 10 against itself", small, small
    yield "separation case: 2 x 2000 against 2 x 2037", *separation_case()


def cdist_sums(pool, ur, ua):
    """The three pair sums of scaled draws [M][P] by cdist, in row blocks on the pool's threads."""
    from scipy.spatial.distance import cdist

    def total(x, y):
        return sum(pool.map(lambda i: float(cdist(x[i:i + BLOCK], y).sum()), range(0, x.shape[0], BLOCK)))

    return total(ur, ua), total(ur, ur), total(ua, ua)


def measure(ctx, pool, name, ref, act, reps):
    P, Mr, Ma = ref.shape[0], ref.shape[1], act.shape[1]
    scale = 1.0 / ref.std(axis=1)
    pairs = Mr * Ma + Mr * (Mr + 1) // 2 + Ma * (Ma + 1) // 2
    dr = _ffi.DeviceBuffer(ctx, ref.nbytes).upload(ref)
    da = _ffi.DeviceBuffer(ctx, act.nbytes).upload(act)
    call = lambda: ctx.energy_distance_dev(dr.ptr, Mr, da.ptr, Ma, P, scale)
    got = call()                                                  # warm-up, and the check
    whole = max(Mr, Ma) <= 4000
    cr, ca = (ref, act) if whole else (ref[:, :2000], act[:, :2000])
    sub = got if whole else ctx.energy_distance(cr, ca, scale)
    exp = _ffi.energy_distance_host(cr, ca, scale)
    assert all(abs(sub[k] - exp[k]) <= 1e-9 * abs(exp[k]) for k in "abc") and abs(sub["e"] - exp["e"]) <= 2e-9 * exp["a"]
    # the baseline's sample: every k-th draw where the pairs are too many
    k = 1
    while (-(-Mr // k)) * (-(-Ma // k)) * 2 * P > BASELINE_WORK:
        k += 1
    ur, ua = np.ascontiguousarray((ref[:, ::k] * scale[:, None]).T), np.ascontiguousarray((act[:, ::k] * scale[:, None]).T)
    base_pairs = ur.shape[0] * ua.shape[0] + ur.shape[0] ** 2 + ua.shape[0] ** 2
    full_pairs = Mr * Ma + Mr * Mr + Ma * Ma
    cdist_sums(pool, ur, ua)
    wall, base = [], []
    for _ in range(reps):                                         # alternating
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        sxy, sxx, syy = cdist_sums(pool, ur, ua)
        base.append((time.perf_counter() - t0) * 1e3 * full_pairs / base_pairs)
    if k == 1:                                                    # the baseline computes the same statistic
        a, b, c = sxy / (Mr * Ma), sxx / (Mr * Mr), syy / (Ma * Ma)
        assert abs((a - b) + (a - c) - got["e"]) <= 1e-9 * 2 * a
    ctx.profile(True)
    kern, launches = {}, {}
    for _ in range(reps):
        ctx.profile_reset()
        call()
        for kn, v in ctx.profile_get().items():
            kern.setdefault(kn, []).append(v["total_ms"])
            launches[kn] = v["launches"]
    ctx.profile(False)
    ctx.profile_reset()
    dr.free()
    da.free()
    pairs_ms = statistics.median(kern["k_energy_pairs"])
    bound_ms = 2.0 * pairs * P / VALU_OPS_PER_S * 1e3             # one subtract and one fma per pair-parameter
    return {"shape": name, "Mr": Mr, "Ma": Ma, "P": P, "pair_parameters": pairs * P, "workspace_bytes": ctx.energy_workspace(Mr, Ma, P),
            "result": got, "call": spread(wall, 3),
            "kernels_ms_per_call": {kn: spread(v) for kn, v in sorted(kern.items())},
            "launches": launches,
            "longest_launch_ms": round(pairs_ms / launches["k_energy_pairs"], 4),
            "valu_bound_ms": round(bound_ms, 4), "k_energy_pairs_fraction_of_fp64_vector_peak": round(bound_ms / pairs_ms, 4),
            "valu_operations_T_per_s": round(2.0 * pairs * P / pairs_ms / 1e9, 2),
            "cdist_baseline": {**spread(base, 1), "threads": THREADS, "block_rows": BLOCK, "every_kth_draw": k,
                               "scaled_by_pair_count": k > 1, "pairs_timed": base_pairs, "pairs_of_the_shape": full_pairs},
            "cdist_over_call": round(statistics.median(base) / statistics.median(wall), 1)}


def edge_errors(ctx):
    """Worst relative error of A, B, C (and of E over 2A) against the host routine over the tests' edge shapes."""
    TI, TJ, PC = _ffi.MCR_ENERGY_TILE_I, _ffi.MCR_ENERGY_TILE_J, _ffi.MCR_ENERGY_CHUNK_P
    sides = lambda T: (1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T - 1)
    worst = {"a": 0.0, "b": 0.0, "c": 0.0, "e_over_2a": 0.0}
    cases = 0
    for P in (1, 2, PC - 1, PC, PC + 1, 2 * PC + 1):
        for Mr in sides(TI):
            for Ma in sides(TJ):
                rng = np.random.default_rng(10007 * Mr + 101 * Ma + P)
                ref, act = rng.normal(size=(P, Mr)) + 1e6 * (cases % 2), rng.normal(size=(P, Ma)) * 1.3 + 0.2 + 1e6 * (cases % 2)
                scale = rng.uniform(0.2, 3.0, size=P)
                got, exp = ctx.energy_distance(ref, act, scale), _ffi.energy_distance_host(ref, act, scale)
                cases += 1
                for k in "abc":
                    if exp[k]:
                        worst[k] = max(worst[k], abs(got[k] - exp[k]) / abs(exp[k]))
                worst["e_over_2a"] = max(worst["e_over_2a"], abs(got["e"] - exp["e"]) / (2 * exp["a"]))
    return {"cases": cases, "gate": 1e-9, **{k: float(f"{v:.3g}") for k, v in worst.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "energy_distance.json"))
    a = ap.parse_args()
    out = {"reps": a.reps, "tile": {"I": _ffi.MCR_ENERGY_TILE_I, "J": _ffi.MCR_ENERGY_TILE_J, "chunk_P": _ffi.MCR_ENERGY_CHUNK_P},
           "max_work": _ffi.MCR_ENERGY_MAX_WORK, "launch_work": _ffi.MCR_ENERGY_LAUNCH_WORK, "shapes": []}
    with _ffi.Context(0) as ctx, ThreadPoolExecutor(THREADS) as pool:
        for name, ref, act in shapes():
            out["shapes"].append(measure(ctx, pool, name, ref, act, a.reps))
        out["worst_error_against_host_routine"] = edge_errors(ctx)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

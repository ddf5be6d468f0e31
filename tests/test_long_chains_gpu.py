"""Tier 3 of the ESS lags on long chains: every FFT size, chain batch and slot count, against the CPU oracle.

Chains of more than 16 384 draws take the lags >= 256 of their first `slots` listed (parameter, kind) pairs from the FFT
tier (mcr_fft.hpp: four-step fp64 FFTs of N = 2^ceil(log2 2n), 2^16 .. 2^22; two chains per complex transform, at most
four transforms per batch, later batches adding to the spectrum) and the rest from the direct rounds of k_acov_long.
A table of AR(1) models walks that plan through each FFT size, odd and even chain counts, one and two batches, the slot
counts 32 .. 2, more listed pairs than slots, and the lengths on either side of where the FFT starts and stops; further
cases cover the workspace limit that halves the slots or drops the FFT, ragged chains, models of several FFT sizes in
one call and the f32 ingest route.  Every case runs on a default context and on one made under MCR_FFT=0 (direct rounds
only); truncation lags and quantiles must equal the oracle's, everything else must agree to 1e-9
(`test_hip_parity.check_summary`), and the profiled launch counts must be the ones the plan makes.

A pair is listed for tier 3 when its first negative rho lies at lag >= 256 (`lag_*` >= 255: the walk accumulated the
lags 1 .. lag_*), and the list holds the pairs in ascending pk = 2p + kind; so the oracle alone tells which pairs the
FFT serves and which go direct.  `python tests/test_long_chains_gpu.py` checks those preconditions and prints each case's
census on a host without a GPU.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest

from test_hip_parity import check_summary

pytestmark = pytest.mark.gpu

ORACLE_THREADS = 16
MIN_CHAINS = 2

# The plan of tier 3 (mcr_api.hip: plan_fft, carve_fft, plan_chunks, launch_diag; mcr_diag.hpp: kLag2).
LAG2 = 256                  # first lag of tier 3
DIRECT_FIRST_END = 16384    # the first direct round takes the lags [256, 16 384), every later one 4x as many
FFT_MIN_N = 16384           # the FFT tier takes chains of more than this many draws ...
FFT_MAX_LOGN = 22           # ... whose N = 2^ceil(log2 2n) is at most 2^22
FFT_CHAIN_BATCH = 4         # complex transforms per batch (two chains each)
WS_ALIGN = 256              # every workspace buffer starts on this boundary


@dataclass(frozen=True)
class FftPlan:
    logN: int
    slots: int              # listed pairs the FFT serves per chunk
    cb: int                 # transforms per batch

    @property
    def geometry(self) -> str:
        return f"{1 << self.logN // 2} x {1 << (self.logN - self.logN // 2)}"


def fft_plan(n: int, C: int, enabled: bool = True) -> FftPlan | None:
    if not enabled or n <= FFT_MIN_N or C < 2:
        return None
    lg = (2 * n - 1).bit_length()
    if lg > FFT_MAX_LOGN:
        return None
    return FftPlan(lg, min(max((1 << 23) >> lg, 2), 32), min((C + 1) // 2, FFT_CHAIN_BATCH))


def fft_bytes(plan: FftPlan, slots: int) -> int:
    """carve_fft's measure: A [slots][cb][N] complex, S [slots][N] real, B [slots][N] complex, each 256-byte aligned."""
    N, off = 1 << plan.logN, 0
    for nbytes in (slots * plan.cb * N * 16, slots * N * 8, slots * N * 16):
        off = -(-off // WS_ALIGN) * WS_ALIGN + nbytes
    return off


def slots_under_limit(plan: FftPlan, limit: int) -> int:
    """plan_chunks: the FFT keeps at most a third of the workspace limit; its slots halve until it does, then it goes."""
    s = plan.slots
    while fft_bytes(plan, s) > limit // 3:
        if s <= 1:
            return 0
        s //= 2
    return s


def fft_launches(C: int, plan: FftPlan | None) -> int:
    """k_fft launches of one chunk: cols + rows_power per batch of 2 cb chains, then rows_spec and cols_out."""
    return 0 if plan is None else 2 * -(-C // (2 * plan.cb)) + 2


def direct_rounds(n: int) -> int:
    rounds, L0 = 0, LAG2
    while L0 < n:
        L0 = DIRECT_FIRST_END if L0 < DIRECT_FIRST_END else 4 * L0
        rounds += 1
    return rounds


def planned_launches(C: int, n: int, plan: FftPlan | None, chunks: int = 1) -> dict:
    """Launches of a call: per chunk, the FFT's and one k_acov_long + k_diag_long_scan per direct round; without the FFT
    and on chains of at most 16 384 draws the fused k_tier3 instead (one launch, profiled as k_acov_long)."""
    if plan is None and n <= DIRECT_FIRST_END:
        return {"k_fft": 0, "k_acov_long": chunks, "k_diag_long_scan": 0}
    r = direct_rounds(n)
    return {"k_fft": chunks * fft_launches(C, plan), "k_acov_long": chunks * r, "k_diag_long_scan": chunks * r}


PROFILED = ("k_fft", "k_acov_long", "k_diag_long_scan")


def profiled(ctx, call):
    ctx.profile(True)
    try:
        ctx.profile_reset()
        r = call()
        prof = ctx.profile_get()
    finally:
        ctx.profile(False)
    return r, {k: prof.get(k, {}).get("launches", 0) for k in PROFILED}


@dataclass(frozen=True)
class Case:
    C: int
    n: int
    P: int
    phi: float
    seed: int
    what: str
    overflow: bool = False  # more listed pairs than FFT slots


CASES = {
    "a": Case(4, 16384, 2, 0.995, 1, "last length before the FFT: fused k_tier3"),
    "b": Case(4, 16385, 2, 0.995, 1, "first FFT length, 256 x 256"),
    "c": Case(3, 32768, 2, 0.995, 1, "largest n of 2^16; odd C: last transform half empty"),
    "d": Case(2, 32769, 2, 0.995, 1, "size step to 2^17, one transform"),
    "e": Case(5, 65537, 2, 0.99, 1, "2^18, odd C: three transforms"),
    "f": Case(9, 131073, 2, 0.99, 1, "2^19, 16 slots: a second batch of one half-empty transform"),
    "g": Case(16, 262145, 2, 0.99, 1, "2^20, 8 slots: two full batches"),
    "h": Case(2, 524289, 3, 0.995, 1, "2^21, 4 slots: 6 listed pairs", overflow=True),
    "i": Case(2, 2097152, 2, 0.99, 1, "2^22, the largest FFT, 2 slots: 4 listed pairs", overflow=True),
    "j": Case(2, 2097153, 2, 0.99, 1, "2^23 > limit: FFT off, direct rounds up to [1 048 576, 4 194 304)"),
}
WS_CASE = Case(4, 60000, 4, 0.995, 1, "workspace limits: slots 1, FFT dropped, chunks sharing 2 slots")
RAGGED = (131073, 140000, 150000)       # diagnose_chains: n = 131 073 (2^19), C = 3, FFT slots capped at 2
RAGGED_PHI, RAGGED_SEED = 0.99, 1
MIXED = ("b", "f", "i")                 # one summarize_models call over three FFT sizes


def ar1(C: int, n: int, P: int, phi: float, seed: int) -> np.ndarray:
    """[P][C][n] AR(1) draws, stationary variance 1, parameter p offset by p."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    x = lfilter([1.0], [1.0, -phi], rng.normal(size=(P, C, n)) * np.sqrt(1 - phi * phi), axis=2)
    x += np.arange(P)[:, None, None]
    return x


def case_draws(case: Case) -> np.ndarray:
    return ar1(case.C, case.n, case.P, case.phi, case.seed)


def ragged_chains() -> list[np.ndarray]:
    x = ar1(len(RAGGED), max(RAGGED), 1, RAGGED_PHI, RAGGED_SEED)[0]
    return [x[c, :m].copy() for c, m in enumerate(RAGGED)]


def pair_lags(exp) -> np.ndarray:
    """lag_* of every pair in list order pk = 2p + kind (kind 0 bulk, 1 tail)."""
    return np.stack([np.asarray(exp["lag_bulk"]), np.asarray(exp["lag_tail"])], axis=1).reshape(-1)


def census(exp, plan: FftPlan | None, slots: int | None = None) -> dict:
    lags = pair_lags(exp)
    listed = [int(pk) for pk in np.flatnonzero(lags >= LAG2 - 1)]
    s = (plan.slots if slots is None else slots) if plan is not None else 0
    return {"pairs": int(lags.size), "listed": len(listed), "fft": listed[:s], "direct": listed[s:],
            "lags": [int(v) for v in lags]}


def assert_precondition(case: Case, exp, what: str) -> dict:
    """What the case is there for, from the oracle alone: every pair reaches tier 3, and an overflow case lists more
    pairs than the FFT has slots."""
    plan = fft_plan(case.n, case.C)
    cen = census(exp, plan)
    assert cen["listed"] == cen["pairs"], (what, cen)
    if case.overflow:
        assert plan is not None and cen["direct"], (what, cen)
    return cen


def oracle_summary(orc, x, layout: str = "pcn") -> dict:
    return orc.summarize_mt(x, layout, threads=ORACLE_THREADS, min_chains=MIN_CHAINS)


class Oracles:
    """Draws and oracle result of each case, made on first use and kept for the module."""

    def __init__(self, orc):
        self.orc = orc
        self.memo = {}

    def _get(self, key, make):
        if key not in self.memo:
            self.memo[key] = make()
        return self.memo[key]

    def case(self, name: str):
        def make():
            x = case_draws(CASES[name])
            return x, oracle_summary(self.orc, x)
        return self._get(name, make)

    def ws(self):
        def make():
            x = case_draws(WS_CASE)
            return x, oracle_summary(self.orc, x)
        return self._get("ws", make)

    def ragged(self):
        def make():
            chains = ragged_chains()
            return chains, self.orc.diag(chains, MIN_CHAINS)
        return self._get("ragged", make)

    def f32_cnp(self):
        def make():
            x = np.ascontiguousarray(self.case("f")[0].astype(np.float32).transpose(1, 2, 0))
            return x, oracle_summary(self.orc, x, "cnp")
        return self._get("f32", make)


@pytest.fixture(scope="module")
def oracles(oracle):
    return Oracles(oracle)


@pytest.fixture(scope="module")
def engines():
    """(context, FFT on): a default context and one made under MCR_FFT=0."""
    from mcmc_ref_hip import _ffi
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCR_FFT", "0")
        direct = _ffi.Context(0)
    fft = _ffi.Context(0)
    yield ((fft, True), (direct, False))
    fft.close()
    direct.close()


def run_engines(engines, x, layout, exp, C, n, what):
    for c, on in engines:
        t = c.upload(x, layout)
        try:
            assert c.params_per_chunk(t) >= t.targs[3], what          # one chunk: the launch counts are per call
            got, launches = profiled(c, lambda: c.summarize(t, min_chains=MIN_CHAINS))
        finally:
            t.free()
        engine = "fft" if on else "direct"
        check_summary(got, exp, what=f"{what} {engine}")
        assert launches == planned_launches(C, n, fft_plan(n, C, on)), (what, engine, launches)


@pytest.mark.parametrize("name", sorted(CASES))
def test_long_chain_case_both_engines(engines, oracles, name):
    case = CASES[name]
    x, exp = oracles.case(name)
    assert_precondition(case, exp, name)
    run_engines(engines, x, "pcn", exp, case.C, case.n, f"case {name}")


def test_f32_cnp_ingest_both_engines(engines, oracles):
    """Case f's draws as f32 in the [C][N][P] layout: the ingest pass widens them into the f64 buffer the FFT reads."""
    case = CASES["f"]
    x, exp = oracles.f32_cnp()
    assert_precondition(case, exp, "f32 cnp")
    run_engines(engines, x, "cnp", exp, case.C, case.n, "case f f32 cnp")


def test_workspace_limit_halves_slots_and_drops_fft(oracles):
    """Under a tight workspace limit the FFT keeps at most a third of it: its slots halve down to 1, then it is dropped;
    and the parameters split into chunks that share the FFT buffers.  Each limit on a fresh context, against the oracle,
    with the chunk count from mcr_plan_chunks and the launches of that many chunks."""
    from mcmc_ref_hip import _ffi
    case = WS_CASE
    x, exp = oracles.ws()
    plan = fft_plan(case.n, case.C)
    assert plan is not None and plan.slots == 32
    assert_precondition(case, exp, "ws")
    limits = {1: 3 * fft_bytes(plan, 1), 0: 3 * fft_bytes(plan, 1) - 3, 2: 3 * fft_bytes(plan, 2)}
    for slots, limit in limits.items():
        assert slots_under_limit(plan, limit) == slots, (slots, limit)
        what = f"ws limit {limit} ({slots} slots)"
        with _ffi.Context(0) as ctx:
            ctx._check(ctx.lib.mcr_set_workspace_limit(ctx.handle, limit))
            t = ctx.upload(x, "pcn")
            try:
                per_chunk = ctx.params_per_chunk(t)
                chunks = -(-case.P // per_chunk)
                assert chunks >= 2, (what, per_chunk)
                got, launches = profiled(ctx, lambda: ctx.summarize(t, min_chains=MIN_CHAINS))
            finally:
                t.free()
        check_summary(got, exp, what=what)
        p = plan if slots else None
        assert launches == planned_launches(case.C, case.n, p, chunks), (what, chunks, launches)
        if slots:                 # every chunk's first listed pair by FFT, the rest of its listed pairs direct
            cen = census({k: exp[k][:per_chunk] for k in ("lag_bulk", "lag_tail")}, plan, slots)
            assert cen["fft"] and cen["direct"], (what, cen)


def test_ragged_chains_fixed_two_slots_both_engines(engines, oracles):
    """mcr_diagnose_chains on three chains whose shortest has 131 073 draws: N = 2^19, an odd chain count, the ragged
    route's FFT slots capped at 2 (one parameter: both its pairs by FFT)."""
    chains, e = oracles.ragged()
    assert min(e["lag_bulk"], e["lag_tail"]) >= LAG2 - 1, e
    n, C = min(RAGGED), len(RAGGED)
    for c, on in engines:
        g, launches = profiled(c, lambda: c.diagnose_chains(chains, MIN_CHAINS))
        engine = "fft" if on else "direct"
        assert (g["lag_bulk"], g["lag_tail"]) == (e["lag_bulk"], e["lag_tail"]), (engine, g, e)
        for k in ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail"):
            assert abs(g[k] - e[k]) <= 1e-9 * max(abs(g[k]), abs(e[k])), (engine, k, g[k], e[k])
        assert launches == planned_launches(C, n, fft_plan(n, C, on)), (engine, launches)


def test_models_of_three_fft_sizes_in_one_call(oracles):
    """One summarize_models call on a fresh context over cases b, f and i (N = 2^16, 2^19, 2^22): models of different
    FFT sizes in flight across the lanes while the context's twiddle cache grows."""
    from mcmc_ref_hip import _ffi
    data = [oracles.case(name) for name in MIXED]
    with _ffi.Context(0) as ctx:
        ts = [ctx.upload(x, "pcn") for x, _ in data]
        try:
            got, launches = profiled(ctx, lambda: ctx.summarize_models(ts, min_chains=MIN_CHAINS))
        finally:
            for t in ts:
                t.free()
    for name, (_, exp), r in zip(MIXED, data, got):
        check_summary(r, exp, what=f"summarize_models case {name}")
    want = {k: 0 for k in PROFILED}
    for name in MIXED:
        case = CASES[name]
        for k, v in planned_launches(case.C, case.n, fft_plan(case.n, case.C)).items():
            want[k] += v
    assert launches == want, launches


if __name__ == "__main__":           # the oracle-only preconditions, on any host
    import sys
    import time
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root), str(root / "mcmc-db_amd")]
    from oracle import oracle as orc
    orc.build()
    oc = Oracles(orc)
    for name, case in CASES.items():
        t0 = time.perf_counter()
        _, exp = oc.case(name)
        dt = time.perf_counter() - t0
        plan = fft_plan(case.n, case.C)
        cen = assert_precondition(case, exp, name)
        geo = "no FFT" if plan is None else (f"N = 2^{plan.logN} ({plan.geometry}), {plan.slots} slots, "
                                             f"{-(-case.C // 2)} transforms in batches of {plan.cb}")
        print(f"{name}: {case.P} x {case.C} x {case.n}, phi {case.phi}: {geo}; {case.what}")
        print(f"   {cen}; launches {planned_launches(case.C, case.n, plan)} / direct "
              f"{planned_launches(case.C, case.n, None)}; oracle {dt:.1f} s")
    t0 = time.perf_counter()
    _, exp = oc.ws()
    plan = fft_plan(WS_CASE.n, WS_CASE.C)
    cen = assert_precondition(WS_CASE, exp, "ws")
    print(f"ws: {WS_CASE.P} x {WS_CASE.C} x {WS_CASE.n}: {cen}; oracle {time.perf_counter() - t0:.1f} s")
    for s in (1, 2):
        print(f"   FFT buffers at {s} slot(s): {fft_bytes(plan, s)} bytes")
    t0 = time.perf_counter()
    _, e = oc.ragged()
    assert min(e["lag_bulk"], e["lag_tail"]) >= LAG2 - 1, e
    plan = fft_plan(min(RAGGED), len(RAGGED))
    print(f"ragged {RAGGED}: lags {e['lag_bulk']} / {e['lag_tail']}, N = 2^{plan.logN} ({plan.geometry}), 2 slots; "
          f"oracle {time.perf_counter() - t0:.1f} s")
    t0 = time.perf_counter()
    _, exp = oc.f32_cnp()
    cen = assert_precondition(CASES["f"], exp, "f32 cnp")
    print(f"f32 cnp: {cen}; oracle {time.perf_counter() - t0:.1f} s")
    print("preconditions hold")

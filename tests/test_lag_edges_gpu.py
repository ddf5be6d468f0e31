"""The ESS truncation lag at every hand-over of the kernels that produce it.

The lag is the work of a relay: tier 1 (k_acov_seg + k_diag_combine) walks the lags 1 .. 63, tier 2 (k_diag_combine2) the
blocks 64 .. 127, 128 .. 191, 192 .. 255, tier 3 the rest -- k_tier3 in 256-lag groups and stages that begin at the lags 256,
768, 2 304, 4 352, ..., or the listed route (k_long_list, k_dev_fill, k_acov_long / the FFTs, k_diag_long_scan) in rounds
[256, 16 384), [16 384, 65 536), ...  An error at a hand-over -- a block that scans one lag too few, a prefix sum that drops
the term at the seam, a stage flag read one group early -- moves the lag of a column whose first negative rho sits exactly
there and of no other.  The recipes of golden/lag_edge_cases.json (lag_edge_cases.py; test_lag_edges_cpu.py holds them to the
oracle and to the full table of seams) put the first negative rho of the bulk ESS at F = seam - 1, seam, seam + 1 on every
route that reaches the seam, with |rho| >= 1e-6 on either side: the tiers' own rho decides, not the guard band's
re-derivation, and every test asserts that `rho_guard_count` does not move.

Gates: those of test_hip_parity.check_summary -- lags and order statistics exact, floating-point fields to 1e-9 of the CPU
oracle.  The oracle runs once per tensor; tiled copies (scaled by powers of two, which changes no rank, z or lag) are
compared with the unscaled case's result.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager

import numpy as np
import pytest

import lag_edge_cases as lec
from test_hip_parity import TIGHT, check_summary, close
from test_long_chains_gpu import LAG2, census, fft_plan

pytestmark = pytest.mark.gpu

MIN_CHAINS = 1
ORACLE_THREADS = 16
CASES = lec.load()
GROUPS = lec.groups(CASES)
KEYS = list(GROUPS)
LONG_KEYS = [k for k in KEYS if k[0] in ("long", "long_round_end")]
LISTED_KEYS = [k for k in KEYS if k[0] in ("short", "one_stage")]          # tiled past kTier3MaxPairs pairs
LISTED_MIN_PARAMS = 1030                                                   # 2 060 pairs > kTier3MaxPairs = 2 048
FORK_KEYS = [k for k in KEYS if k[0] in ("segments", "multi_stage")]       # tiled into the fork window
FORK_WINDOW = (2e6, 8e6)                                                   # param-draws of a lone call that forks (mcr_api.hip)
DIAG_FIELDS = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")


def group_id(key) -> str:
    return f"{key[0]}-C{key[1]}-N{key[2]}"


@pytest.fixture(scope="module")
def ctx():
    from mcmc_ref_hip import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def engines():
    """(context, FFT on): a default context and one made under MCR_FFT=0, as in test_long_chains_gpu.py."""
    from mcmc_ref_hip import _ffi
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MCR_FFT", "0")
        direct = _ffi.Context(0)
    fft = _ffi.Context(0)
    yield ((fft, True), (direct, False))
    fft.close()
    direct.close()


class Oracles:
    """Draws and oracle results of each (route, C, N) tensor, made on first use, kept for the module and never written."""

    def __init__(self, orc):
        self.orc = orc
        self.memo = {}

    def group(self, key):
        if key not in self.memo:
            x = lec.tensor(GROUPS[key])
            exp = self.orc.summarize_mt(x, "pcn", threads=ORACLE_THREADS, min_chains=MIN_CHAINS)
            for p, case in enumerate(GROUPS[key]):                 # what the case is there for, from the oracle alone
                assert int(exp["lag_bulk"][p]) + 1 == case["F"] and int(exp["lag_tail"][p]) == case["lag_tail"], case
            self.memo[key] = (x, exp)
        return self.memo[key]

    def diag(self, key):
        if ("diag", key) not in self.memo:
            x, _ = self.group(key)
            with ThreadPoolExecutor(ORACLE_THREADS) as pool:
                self.memo["diag", key] = list(pool.map(lambda xp: self.orc.diag(list(xp), MIN_CHAINS), x))
        return self.memo["diag", key]


@pytest.fixture(scope="module")
def oracles(oracle):
    return Oracles(oracle)


@contextmanager
def guard_untouched(*contexts):
    """The decisions inside are the tiers' own: no lag is re-derived by the guard band."""
    before = [c.rho_guard_count() for c in contexts]
    yield
    assert [c.rho_guard_count() for c in contexts] == before


def tiled(x: np.ndarray, copies: int) -> np.ndarray:
    """[copies * P][C][N]: copy k is x times 2^(k - copies // 2), exact; parameter k * P + p is case p."""
    scale = np.ldexp(1.0, np.arange(copies) - copies // 2)
    return np.ascontiguousarray((x[None] * scale[:, None, None, None]).reshape(-1, *x.shape[1:]))


def check_copies(got, exp, cases, copies: int, what: str):
    """Every copy's lags are the case's and its ESS and R-hat the oracle's of the unscaled case."""
    P = len(cases)
    for k in range(copies):
        for p, case in enumerate(cases):
            i = k * P + p
            assert int(got["lag_bulk"][i]) == case["F"] - 1, (what, k, case, int(got["lag_bulk"][i]))
            assert int(got["lag_tail"][i]) == case["lag_tail"], (what, k, case, int(got["lag_tail"][i]))
            for f in DIAG_FIELDS:
                assert close(got[f][i], exp[f][p], TIGHT), (what, k, case, f, got[f][i], exp[f][p])


def same_bits(a: dict, b: dict, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def lone_and_enqueued(ctx, x: np.ndarray, what):
    """One synchronous call with nothing else in flight, then 8 enqueued calls on the same uploaded tensor: same bits."""
    t = ctx.upload(x, "pcn")
    try:
        lone = ctx.summarize(t, min_chains=MIN_CHAINS)
        bufs = [ctx.enqueue(t, min_chains=MIN_CHAINS) for _ in range(8)]
        ctx.wait()
    finally:
        t.free()
    for q in bufs:
        same_bits(lone, q.result(), what)
    return lone


@pytest.mark.parametrize("key", KEYS, ids=group_id)
def test_batched_route_tensor(ctx, oracles, key):
    """The cases of a route side by side in one call: pairs that end at F - 1, F and F + 1 share k_tier3's `decided` words
    and the tier-3 list."""
    x, exp = oracles.group(key)
    with guard_untouched(ctx):
        got = ctx.summarize(x, "pcn", min_chains=MIN_CHAINS)
    check_summary(got, exp, what=group_id(key))


@pytest.mark.parametrize("key", KEYS, ids=group_id)
def test_one_parameter_per_call_lone_and_enqueued(ctx, oracles, key):
    x, exp = oracles.group(key)
    with guard_untouched(ctx):
        for p, case in enumerate(GROUPS[key]):
            got = lone_and_enqueued(ctx, x[p:p + 1], case)
            assert (int(got["lag_bulk"][0]), int(got["lag_tail"][0])) == (case["F"] - 1, case["lag_tail"]), case
            check_summary(got, {k: v[p:p + 1] for k, v in exp.items()}, what=f"{group_id(key)} F={case['F']} alone")


@pytest.mark.parametrize("key", FORK_KEYS, ids=group_id)
def test_lone_call_that_forks_the_kinds_over_two_streams(ctx, oracles, key):
    """A lone call of 2 M .. 8 M param-draws in one chunk runs the bulk and the folded half of tiers 1 and 2 as launches of
    their own (kind_sel 0 / 1) on two streams; one parameter is far below that, so the route's tensor is tiled up to it."""
    x, exp = oracles.group(key)
    P, C, N = x.shape
    copies = -(-int(FORK_WINDOW[0]) // (P * C * N))
    xt = tiled(x, copies)
    assert FORK_WINDOW[0] <= xt.size <= FORK_WINDOW[1], xt.shape
    t = ctx.upload(xt, "pcn")
    try:
        assert ctx.params_per_chunk(t) >= xt.shape[0]
    finally:
        t.free()
    with guard_untouched(ctx):
        got = lone_and_enqueued(ctx, xt, group_id(key))
    check_copies(got, exp, GROUPS[key], copies, f"{group_id(key)} forked")


@pytest.mark.parametrize("key", KEYS, ids=group_id)
def test_diagnose_chains(ctx, oracles, key):
    x, _ = oracles.group(key)
    exps = oracles.diag(key)
    with guard_untouched(ctx):
        for case, xp, e in zip(GROUPS[key], x, exps):
            g = ctx.diagnose_chains(list(xp), MIN_CHAINS)
            assert (e["lag_bulk"], e["lag_tail"]) == (case["F"] - 1, case["lag_tail"]), (case, e)
            assert (g["lag_bulk"], g["lag_tail"]) == (e["lag_bulk"], e["lag_tail"]), (case, g)
            for f in DIAG_FIELDS:
                assert close(g[f], e[f], TIGHT), (case, f, g[f], e[f])


@pytest.mark.parametrize("key", LISTED_KEYS, ids=group_id)
def test_listed_route_on_chains_of_at_most_16384_draws(ctx, oracles, key):
    """More than kTier3MaxPairs = 2 048 pairs in a chunk: tier 3 goes through k_long_list, k_dev_fill, one round of
    k_acov_long and k_diag_long_scan instead of k_tier3."""
    x, exp = oracles.group(key)
    cases = GROUPS[key]
    copies = -(-LISTED_MIN_PARAMS // len(cases))
    xt = tiled(x, copies)
    t = ctx.upload(xt, "pcn")
    try:
        assert ctx.params_per_chunk(t) >= xt.shape[0] > 1024, "one chunk of more than 2 048 pairs"
        with guard_untouched(ctx):
            got = ctx.summarize(t, min_chains=MIN_CHAINS)
    finally:
        t.free()
    assert max(c["F"] for c in cases) > LAG2, "no case of the tensor reaches tier 3"
    check_copies(got, exp, cases, copies, f"{group_id(key)} listed")


@pytest.mark.parametrize("key", LONG_KEYS, ids=group_id)
def test_long_chains_fft_and_direct_rounds(engines, oracles, key):
    x, exp = oracles.group(key)
    with guard_untouched(*(c for c, _ in engines)):
        got = {on: c.summarize(x, "pcn", min_chains=MIN_CHAINS) for c, on in engines}
    for on, r in got.items():
        check_summary(r, exp, what=f"{group_id(key)} {'fft' if on else 'direct'}")
    assert np.array_equal(got[True]["lag_bulk"], got[False]["lag_bulk"])
    assert np.array_equal(got[True]["lag_tail"], got[False]["lag_tail"])


def test_long_chains_more_listed_pairs_than_fft_slots(engines, oracles):
    """The first `slots` listed pairs take their lags from the FFT and the rest from the direct rounds, in one call: the
    cases around lag 256 and 512 on both sides of that line."""
    key = next(k for k in LONG_KEYS if k[0] == "long")
    x, exp = oracles.group(key)
    cases = GROUPS[key]
    _, C, N = x.shape
    plan = fft_plan(N, C)
    assert plan is not None
    listed_per_copy = census(exp, plan)["listed"]
    assert listed_per_copy >= 4, census(exp, plan)
    copies = plan.slots // listed_per_copy + 2
    xt = tiled(x, copies)
    exp_t = {k: np.tile(exp[k], copies) for k in ("lag_bulk", "lag_tail")}
    cen = census(exp_t, plan)
    assert cen["fft"] and cen["direct"], cen
    fft_F = {cases[pk // 2 % len(cases)]["F"] for pk in cen["fft"] if pk % 2 == 0}
    direct_F = {cases[pk // 2 % len(cases)]["F"] for pk in cen["direct"] if pk % 2 == 0}
    assert fft_F == direct_F == {c["F"] for c in cases if c["F"] >= LAG2}, (fft_F, direct_F)   # every seam case by both engines
    for c, on in engines:
        t = c.upload(xt, "pcn")
        try:
            assert c.params_per_chunk(t) >= xt.shape[0]            # one chunk, one list
            with guard_untouched(c):
                got = c.summarize(t, min_chains=MIN_CHAINS)
        finally:
            t.free()
        check_copies(got, exp, cases, copies, f"{group_id(key)} overflow {'fft' if on else 'direct'}")
